"""The design of tests/_positions.py, checked without a GPU: the restated geometry and what each pinned shape reaches in it, the
coverage of the permutations, the conditions under which the planted answers ARE the answers (asserted from the inputs: a blocked
fp32 matrix product, no O(n^2) oracle), and a rehearsal of every GPU test body against a stand-in device that answers from the CPU
oracle at a reduced n.  The rehearsal proves the expectations and the comparison code; it proves nothing about the kernels."""
import numpy as np
import pytest

import _positions as P

REHEARSAL_N = 715      # odd (a single row besides the twins), a ragged last mask word of 11 rows, three 256-row tiles


# ---- 1b: the restated geometry and what the shapes reach in it ----------------------------------------------------------------
def test_restated_plan_numbers_filter_tiles_around_the_sample_tiles():
    for n in (P.N_A, P.N_B, P.N_S, P.N_M, 150_000, 1_000_000, 12_500_000):
        for tile_rows in (P.TILE_ROWS, P.F32_TILE_ROWS):
            p = P.plan(n, tile_rows=tile_rows)
            assert p["stride"] >= 2 and p["n_sample_tiles"] + p["n_filter_tiles"] == p["n_tiles"]
            ft = P.filter_tiles(p)
            assert len(ft) == p["n_filter_tiles"]
            assert ft == [P.filter_tile(sel, p["stride"]) for sel in range(len(ft))]
            assert [t for t in range(p["n_tiles"]) if P.is_sample_tile(t, p["stride"])] == [s * p["stride"] for s in range(p["n_sample_tiles"])]
    # the plan of test_parity_sweep's largest shape, worked by hand from scan_api.cpp:34-50: 586 tiles, 8192 sample rows wanted
    # = 32 tiles, stride 18, 33 sample tiles
    p = P.plan(150_000)
    assert (p["n_tiles"], p["stride"], p["n_sample_tiles"], p["n_filter_tiles"]) == (586, 18, 33, 553)
    assert P.plan(P.N_X)["stride"] == 1      # a shard of 8 321 rows is ALL sample tiles: no filter kernel would run on it


def test_resident_shapes_end_as_the_design_says():
    """Shape A: a last unit of one tile, that tile a filter tile whose last 64-row block holds one row.  Shape B: the last tile
    is a sample tile (and ragged).  Both: 32 row streams at 1024 queries per slice, 160 tiles or more, a ragged last slice."""
    a, b = P.plan(P.N_A), P.plan(P.N_B)
    ua, last_a = P.units(a)
    assert last_a == 1 and a["n_filter_tiles"] % 2 == 1
    assert not P.is_sample_tile(a["n_tiles"] - 1, a["stride"]) and P.filter_tiles(a)[-1] == a["n_tiles"] - 1
    assert P.N_A % P.BLOCK_ROWS == 1 and ua[-1] == (P.N_A - 1, P.N_A - 1)
    ub, last_b = P.units(b)
    assert P.is_sample_tile(b["n_tiles"] - 1, b["stride"]) and last_b == 2 and P.N_B % P.TILE_ROWS not in (0, 1)
    assert ub[-1][1] == (b["n_tiles"] - 1) * P.TILE_ROWS - 1          # the last filter row lies in front of the sample tile
    for n, p in ((P.N_A, a), (P.N_B, b)):
        r = P.resident(p, P.SLICE_QUERIES)
        assert r == dict(use=True, n_qt=8, n_streams=32, n_units=(p["n_filter_tiles"] + 1) // 2)
        assert n >= 32 * 5 * 256 and n % P.SLICE_QUERIES != 0
        # 256-row strips per stream (a stream's units are stream, stream + 32, ...: scan_i8d_kernel.h:50): four or more, so the
        # pacing of sibling workgroups at every fourth strip is reached
        assert 2 * (r["n_units"] // r["n_streams"]) >= 4
        last = P.resident(p, n % P.SLICE_QUERIES)                       # the ragged last slice: fewer query tiles, more streams
        assert last["use"] and last["n_qt"] < 8
    for name in P.RESIDENT_FORMS:
        assert P.FORMS[name]["n"] in (P.N_A, P.N_B) and P.FORMS[name]["dim"] % 128 == 0 and P.FORMS[name]["dim"] <= 768


def test_every_form_has_filter_tiles_and_a_ragged_end():
    for f in P.FORMS.values():
        n, dim = f["n"], f["dim"]
        if f.get("path", 0) == 1:
            continue
        p = P.form_plan(f)
        assert n >= P.MFMA_MIN_ROWS and n > 16384 and dim % 4 == 0, f["name"]          # (n > 16384: never the fused small scan)
        assert p["stride"] >= 2 and p["n_filter_tiles"] >= 32, (f["name"], p)
        assert n % p["tile_rows"] != 0 and n % 32 != 0, f["name"]
        if "masked" in f["cases"]:
            assert n // 2 >= P.MASK_MIN_ALLOWED, f["name"]
        if "medium" in f["cases"]:
            assert dim >= 384
        if f["tier"] == 1:
            assert dim % 64 == 0 and dim >= 256 and f["shadow"] in ("i8", "both")
            if f["name"] not in P.RESIDENT_FORMS:
                assert dim % 128 != 0                                               # half tiles: no resident form exists
        if f["tier"] in (2, 3):
            assert dim % 16 == 0
        if f["tier"] == 4:
            assert "FLAG_F32_FILTER" in f.get("flags", ()) or dim % 16 != 0
    assert P.call_ranges(P.N_S, 128)[-1] == (P.N_S - 128, 128) and len(P.call_ranges(P.N_S, 128)) == 131
    assert P.call_ranges(300, None) == [(0, 300)]
    assert len(P.call_ranges(P.N_S, 64)) == 261 and P.call_ranges(P.N_S, 64)[-1] == (P.N_S - 64, 64)
    for name in ("bf16n_192_q128", "bf16n_192_q64", "l2_bf16n_192_q64"):       # the narrow kernel's rule, scan_bf16_kernel.hip:1335-1358
        f = P.FORMS[name]
        assert f["dim"] % 32 == 0 and f["dim"] >= 64 and not 256 <= f["dim"] <= 512 and f["shadow"] == "bf16" and not f.get("flags")
        assert f["per_call"] <= (128 if f.get("metric", "cosine") == "cosine" else 64)


# ---- 1c: coverage, on the test's own indices ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sorted({f["n"] for f in P.FORMS.values() if f.get("path", 0) == 0}))
def test_permutations_reach_every_row_pair_and_tile_edge(n):
    """Every row is a winner; every (row mod 64, query mod 128) and every (row mod 256, slice-local query tile) pair occurs; the
    first / last row of every 256-row tile — and so of every unit — is the winner of a query in slot 0 / slot 127.  The
    structured permutation reaches all of it alone; the affine one is a second, independent pattern over the same rows."""
    first, second = P.perm_for("self", n), P.perm_for("self2", n)
    c = P.assert_coverage([first], n)
    assert c["n_pins"] == 2 * (-(-n // 256)) - (n % 256 == 1)
    assert np.array_equal(np.sort(second), np.arange(n)) and not np.array_equal(first, second)
    inv = np.empty(n, np.int64); inv[first] = np.arange(n)
    for lo, hi in P.units(P.plan(n))[0]:
        assert inv[lo] % 128 == 0 and (hi == lo or inv[hi] % 128 == 127), (lo, hi)
    assert np.array_equal(first, P.perm_for("twins", n))               # seeded: the same bijection every time


def test_twin_mask_splits_every_pair_and_every_boundary_word(oracle):
    for n in (P.N_A, P.N_B, P.N_M, REHEARSAL_N):
        twin = np.full(n, -1, np.int64)
        h = n // 2
        sigma = np.random.default_rng(P.SEED + 1).permutation(h)
        twin[h:2 * h] = sigma; twin[sigma] = np.arange(h, 2 * h)
        keep = P.twin_mask(n, twin)
        words = P.boundary_words(n)
        assert {0, 1, n // 32 - 1} <= set(words) and (n % 32 <= 1 or n // 32 in words)
        for w in words:
            bits = keep[32 * w:min(n, 32 * w + 32)]
            assert bits.any() and not bits.all(), (n, w)
        assert int(keep.sum()) == n - h
    _, twin, tie_rank, _ = P.twins_corpus(oracle, REHEARSAL_N, 64)
    assert (twin[twin[twin >= 0]] == np.flatnonzero(twin >= 0)).all() and np.array_equal(np.sort(tie_rank), np.arange(REHEARSAL_N))


# ---- 1a: the planted answers are the answers -------------------------------------------------------------------------------
def _max_other_cosine(queries, corpus, own):
    """max over rows i != own[j] of cos(queries[j], corpus[i]) for every j: blocked fp32 products (error ~1e-5, the margins
    asserted on it are 0.05 and more)."""
    import torch
    c = torch.from_numpy(np.array(corpus)); c = c / c.norm(dim=1, keepdim=True)
    out = np.empty(len(queries), np.float32)
    for j0 in range(0, len(queries), 4096):
        q = torch.from_numpy(np.array(queries[j0:j0 + 4096])); q = q / q.norm(dim=1, keepdim=True)
        s = q @ c.T
        s[torch.arange(len(q)), torch.from_numpy(np.array(own[j0:j0 + 4096]))] = -2.0
        out[j0:j0 + 4096] = s.max(dim=1).values.numpy()
    return out


SELF_SHAPES = sorted({(f["n"], f["dim"]) for f in P.FORMS.values()})


@pytest.mark.parametrize("n,dim", SELF_SHAPES)
def test_no_other_row_comes_near_a_self_match(oracle, n, dim):
    """Off-diagonal cosine of the corpus below 0.8 (threshold of the planted cases: 0.9): the self, twins and masked answers
    hold exactly the planted rows.  The twins corpus is the same rows (its second half copies of its first)."""
    corpus, bits = P.self_corpus(oracle, n, dim)
    m = _max_other_cosine(corpus, corpus, np.arange(n))
    print("largest off-diagonal cosine", n, dim, float(m.max()))
    assert m.max() < 0.8
    assert (bits.view(np.float32) >= 0.9).all()
    tw = P.twins_corpus(oracle, n, dim)[0]
    h = n // 2
    assert np.array_equal(tw[:h], corpus[:h]) and np.array_equal(tw[2 * h:], corpus[2 * h:])
    assert np.array_equal(np.sort(tw[h:2 * h].view(np.uint32), axis=0), np.sort(corpus[:h].view(np.uint32), axis=0))


@pytest.mark.parametrize("n,dim", sorted({(f["n"], f["dim"]) for f in P.FORMS.values() if "medium" in f["cases"]}))
def test_planted_row_is_rank_one_of_every_medium_query(oracle, n, dim):
    corpus, _ = P.self_corpus(oracle, n, dim)
    q = P.medium_queries(oracle, n, dim)                               # per row; a case permutes them
    own = np.array([oracle.cosine(q[j], corpus[j]) for j in range(0, n, 97)])
    assert np.abs(own - P.MEDIUM_C).max() < 1e-6
    m = _max_other_cosine(q, corpus, np.arange(n))
    print("largest similarity of another row", n, dim, float(m.max()))
    assert m.max() < P.MEDIUM_C - 0.05
    full = P.medium_full_queries(n)
    assert len(full) == 24 and {0, 127, 128, 1023, n - 1} <= set(full)


# ---- 4: the rehearsal -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,case", P.PARAMS)
def test_rehearsal_against_the_oracle_stand_in(oracle, form, case):
    f = P.FORMS[form]
    c = P.make_case(oracle, f, case, n=REHEARSAL_N)
    res = P.drive(c, f, lambda q0, cnt: P.stand_in(oracle, c, f, q0, cnt))
    P.verify(c, res, f)
    assert c.known[:, 0].all() and (case != "medium" or c.known[c.full].all())


def test_comparison_reports_the_first_lost_position(oracle):
    """The comparison can fail, and names the geometry of what it lost: a result without one planted row, one with a row id that
    lost its high word, one whose padding was left as the buffer held it."""
    f = dict(P.FORMS["f32_100_row_base"])
    c = P.make_case(oracle, f, "self", n=REHEARSAL_N)
    good = P.stand_in(oracle, c, f)
    P.verify(c, good, f)
    lost = P.Result(good.counts.copy(), good.rows.copy(), good.scores.copy(), good.dist.copy(), good.diag)
    lost.counts[300] = 0; lost.rows[300, 0] = -1; lost.scores[300, 0] = -np.inf; lost.dist[300, 0] = np.inf
    with pytest.raises(AssertionError) as e:
        P.verify(c, lost, f)
    assert e.value.args[0][0] == "count" and e.value.args[0][2] == P.where(c, 300, 128) and e.value.args[0][2]["tile"] == c.perm[300] // 128 and e.value.args[0][2]["planted_row"] == c.perm[300]
    low = P.Result(good.counts, good.rows & 0xFFFFFFFF, good.scores, good.dist, good.diag)
    with pytest.raises(AssertionError) as e:
        P.verify(c, low, f)
    assert e.value.args[0][0] == "rows"
    dirty = P.Result(good.counts, good.rows, good.scores.copy(), good.dist, good.diag)
    dirty.scores[5, 7] = 0.0
    with pytest.raises(AssertionError) as e:
        P.verify(c, dirty, f)
    assert e.value.args[0][0] == "score padding"
    with pytest.raises(AssertionError):
        P.verify(c, P.Result(good.counts, good.rows, good.scores, good.dist, dict(good.diag, exact_fallback_queries=1)), f)
