"""The general scan across the dimension lattice on the device (tests/_dim_lattice.py has the design, tests/stress_dims.py the
harness): one test per class over that class's dims — every form and both metrics of each dim through the harness functions
on the shared context — the harness as a whole, the refusals at the lattice's boundaries, and the same dims through
vector_scan_v1, whose mirror picks its own shadows and layout from dim."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _dim_lattice as dl
import stress_dims
from _dim_lattice import SCAN_COSINE, SCAN_L2
from yams_amd import _lib

pytestmark = pytest.mark.gpu

HARNESS_CASES = stress_dims.DEFAULT_CASES      # six rounds over the 23 cells


def _run_dim(acc, oracle, cls, dim):
    timing = {}
    for metric, forms, l2_acc, limit, d in stress_dims.scripted_draws(cls, dim):
        msg, infos = stress_dims.check_forms(oracle, acc, d, forms, limit)
        print("LATTICE " + json.dumps({"cls": cls, "dim": dim, "metric": metric, "forms": infos}))
        assert msg is None, (cls, dim, metric, msg, infos)
        for form, info in infos.items():
            want = dl.route(dict(d, form=form, **dl.form_fields(cls, form, metric, l2_acc)), None)
            assert info["diag"]["path"] == want[0] and (want[1] is None or info["diag"]["filter_tier"] == want[1]), (form, info)
            timing[(metric, form)] = info["diag"]["filter_tier"]
    return timing


@pytest.mark.parametrize("dim", dl.CLASSES["A"])
def test_class_a_dim_not_a_multiple_of_4_takes_the_scalar_walk(acc, oracle, dim):
    _run_dim(acc, oracle, "A", dim)


@pytest.mark.parametrize("dim", dl.CLASSES["B"])
def test_class_b_misaligned_base_takes_the_exhaustive_path(acc, oracle, dim):
    _run_dim(acc, oracle, "B", dim)


@pytest.mark.parametrize("dim", dl.CLASSES["C"])
def test_class_c_f32_tier_partial_last_slab(acc, oracle, dim):
    tiers = _run_dim(acc, oracle, "C", dim)
    assert set(tiers.values()) == {_lib.TIER_F32}


@pytest.mark.parametrize("dim", dl.CLASSES["D"])
def test_class_d_bf16_16_wide_slabs(acc, oracle, dim):
    tiers = _run_dim(acc, oracle, "D", dim)
    assert tiers[(SCAN_COSINE, "default")] == tiers[(SCAN_L2, "default")] == _lib.TIER_BF16
    assert tiers[(SCAN_COSINE, "split")] == tiers[(SCAN_L2, "split")] == _lib.TIER_SPLIT


@pytest.mark.parametrize("dim", dl.CLASSES["E"])
def test_class_e_bf16_32_wide_slabs_at_every_form_edge(acc, oracle, dim):
    tiers = _run_dim(acc, oracle, "E", dim)
    for metric in (SCAN_COSINE, SCAN_L2):
        assert [tiers[(metric, f)] for f in ("default", "wide", "split", "bare")] == [_lib.TIER_BF16, _lib.TIER_BF16, _lib.TIER_SPLIT, _lib.TIER_BF16]


@pytest.mark.parametrize("dim", dl.CLASSES["F"])
def test_class_f_int8_tier_both_layouts_and_the_resident_form(acc, oracle, dim):
    tiers = _run_dim(acc, oracle, "F", dim)
    assert all(t == _lib.TIER_I8 for (metric, _), t in tiers.items() if metric == SCAN_COSINE), tiers
    assert ((SCAN_COSINE, "rotated") in tiers) == (dl.i8_rotation_window(dim) != 0)
    assert ((SCAN_COSINE, "resident") in tiers) == (dim % 128 == 0 and dim <= 768)


def test_harness_as_a_whole():
    """tests/stress_dims.py in its own process, on its own context: the case count, no mismatch, every counter reached."""
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "stress_dims.py"), "--cases", str(HARNESS_CASES)],
                       capture_output=True, text=True, timeout=280)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-2000:])
    res = json.loads(p.stdout.strip().splitlines()[-1])
    print("STRESS_DIMS " + json.dumps(res))
    assert res["cases"] == HARNESS_CASES and res["mismatches"] == 0 and not res["dry_run"]
    missing = [name for name in stress_dims.required_counters() if res["counters"].get(name, 0) < 1]
    assert not missing, missing


# ---- refusals at the lattice's boundaries -----------------------------------------------------------------------------------
class _Guarded:
    """`nbytes` of device memory between two 256-byte guard words, all of it 0xA5: untouched() says nothing was written."""
    def __init__(self, acc, nbytes):
        self.acc, self.nbytes = acc, nbytes
        self.buf = acc.alloc(nbytes + 512)
        self.buf.upload(np.full(nbytes + 512, 0xA5, np.uint8))
        self.ptr = self.buf.ptr + 256

    def untouched(self):
        return bool((self.buf.download(np.uint8, self.nbytes + 512) == 0xA5).all())


def _refused(status, fn, *bufs):
    with pytest.raises(_lib.AccelError) as e:
        fn()
    assert e.value.status == status, (e.value.status, _lib.STATUS_NAMES.get(e.value.status))
    for b in bufs:
        assert b.untouched()


def test_refusals_at_the_boundaries_leave_the_outputs_untouched(acc, oracle):
    held = []            # every device buffer of the test, freed in the end: the context is the session's

    def keep(b):
        held.append(b.buf if isinstance(b, _Guarded) else b)
        return b
    try:
        n = 4096
        # the bf16 shadow needs dim % 4 == 0
        rows = keep(acc.to_device(oracle.synth_rows(3, 0, n, 30)))
        g_b, g_n = keep(_Guarded(acc, n * 30 * 2)), keep(_Guarded(acc, n * 4))
        _refused(_lib.YAMS_ERR_INVALID_ARG, lambda: acc.build_shadow_device(rows.ptr, n, 30, g_b.ptr, g_n.ptr), g_b, g_n)
        # the int8 shadow needs dim % 64 == 0 and dim >= 256
        for dim in (192, 288):
            rows = keep(acc.to_device(oracle.synth_rows(3, 0, n, dim)))
            g_8, g_m = keep(_Guarded(acc, _lib.i8_shadow_rows(n) * dim)), keep(_Guarded(acc, (n + 15) // 16 * 8))
            for fl in (0, _lib.I8_ROTATED):
                _refused(_lib.YAMS_ERR_INVALID_ARG if fl == 0 or dim >= 256 else _lib.YAMS_ERR_UNSUPPORTED,
                         lambda: acc.build_shadow_i8_device(rows.ptr, n, dim, g_8.ptr, g_m.ptr, i8_flags=fl), g_8, g_m)
        # no rotated layout above 4096; unknown layout bits
        dim = 4160
        corpus = oracle.synth_rows(3, 0, n, dim)
        rows = keep(acc.to_device(corpus))
        g_8, g_m = keep(_Guarded(acc, _lib.i8_shadow_rows(n) * dim)), keep(_Guarded(acc, (n + 15) // 16 * 8))
        _refused(_lib.YAMS_ERR_UNSUPPORTED, lambda: acc.build_shadow_i8_device(rows.ptr, n, dim, g_8.ptr, g_m.ptr, i8_flags=_lib.I8_ROTATED), g_8, g_m)
        _refused(_lib.YAMS_ERR_INVALID_ARG, lambda: acc.build_shadow_i8_device(rows.ptr, n, dim, g_8.ptr, g_m.ptr, i8_flags=2), g_8, g_m)
        _refused(_lib.YAMS_ERR_INVALID_ARG, lambda: acc.build_shadow_i8_device(rows.ptr, n, dim, g_8.ptr, g_m.ptr, i8_flags=_lib.I8_ROTATED | 4), g_8, g_m)
        # a scan whose view names the rotated layout at 4160, or unknown bits: refused before anything is written
        d8, dm = keep(acc.alloc(_lib.i8_shadow_rows(n) * dim)), keep(acc.alloc((n + 15) // 16 * 8))
        acc.build_shadow_i8_device(rows.ptr, n, dim, d8.ptr, dm.ptr)
        nq, k = 17, 10
        q = keep(acc.to_device(oracle.synth_rows(3, 1 << 40, nq, dim)))
        for fl in (_lib.I8_ROTATED, 2):
            view = acc.corpus_view(rows.ptr, n, dim, rows_i8_ptr=d8.ptr, rows_i8_meta_ptr=dm.ptr, i8_flags=fl)
            g_s, g_r, g_c, g_d = keep(_Guarded(acc, nq * k * 4)), keep(_Guarded(acc, nq * k * 8)), keep(_Guarded(acc, nq * 4)), keep(_Guarded(acc, nq * k * 4))
            _refused(_lib.YAMS_ERR_INVALID_ARG, lambda: acc.scan_topk_device(view, q.ptr, nq, k, -1.0, SCAN_COSINE, g_s.ptr, g_r.ptr, g_c.ptr, g_d.ptr),
                     g_s, g_r, g_c, g_d)
        # ... and the same view with the plain layout answers, on the int8 tier
        view = acc.corpus_view(rows.ptr, n, dim, rows_i8_ptr=d8.ptr, rows_i8_meta_ptr=dm.ptr)
        r = acc.scan_topk(view, oracle.synth_rows(3, 1 << 40, nq, dim), k, -1.0)
        assert r.diag["filter_tier"] == _lib.TIER_I8 and r.diag["path"] == 0
        rows_o, sims_o, _, _ = oracle.scan_cosine(corpus, oracle.synth_rows(3, 1 << 40, nq, dim)[5], k)
        assert np.array_equal(r.rows[5], rows_o) and np.array_equal(r.scores[5].view(np.uint32), sims_o.view(np.uint32))
    finally:
        for b in held:
            b.free()


# ---- what the harness's row counts cannot reach: a filter under an allow-mask, and the row counts of the planner's fault -------
@pytest.mark.parametrize("d,forms", stress_dims.masked_draws(), ids=lambda v: "%d-%d" % (v["dim"], v["metric"]) if isinstance(v, dict) else "")
def test_class_d_16_wide_slabs_under_a_dense_mask(acc, oracle, d, forms):
    """An allow-mask that admits fewer than 16384 rows is gathered and scored exhaustively, so no masked case of the lattice's
    4096 .. 5001 rows meets a filter: 21 000 rows of which ~17 600 are allowed, the 16-wide-slab kernel in both forms."""
    msg, infos = stress_dims.check_forms(oracle, acc, d, forms, 6)
    print("LATTICE_MASKED " + json.dumps({"dim": d["dim"], "metric": d["metric"], "forms": infos}))
    assert msg is None, (d, msg, infos)
    assert [infos[f]["diag"]["filter_tier"] for f in forms] == [_lib.TIER_BF16, _lib.TIER_SPLIT]
    assert all(i["diag"]["path"] == 0 and 17 * 16384 <= i["diag"]["rows_visited"] < 17 * 21_000 for i in infos.values())


@pytest.mark.parametrize("d,forms", stress_dims.filter_pass_draws(), ids=lambda v: str(v["dim"]) if isinstance(v, dict) else "")
def test_class_f_half_tile_filter_pass(acc, oracle, d, forms):
    """The int8 half-tile kernel's k loop decides an answer only in its FILTER pass, which needs filter tiles: 16 700 rows
    (every second tile), slab counts 5, 7, 13 and 17."""
    msg, infos = stress_dims.check_forms(oracle, acc, d, forms, 6)
    print("LATTICE_FILTER_PASS " + json.dumps({"dim": d["dim"], "forms": infos}))
    assert msg is None, (d, msg, infos)
    assert all(i["diag"]["filter_tier"] == _lib.TIER_I8 and i["diag"]["path"] == 0 for i in infos.values()), infos


@pytest.mark.parametrize("d,forms", stress_dims.planner_draws(), ids=lambda v: "%d-%d" % (v["n"], v["k"]) if isinstance(v, dict) else "")
def test_padding_groups_of_a_ragged_last_tile_do_not_send_every_query_to_the_exhaustive_pass(acc, oracle, d, forms):
    """4097 .. 4351 rows on the 256-row tiles, k <= 10: every tile is a sample tile, the padding behind the last row forms
    groups of maximum -inf, and the plan counted them as ranks a finite threshold could use — the threshold was -inf, the
    lists were cut at 4096 < n and EVERY query fell back (make_plan, scan_api.cpp).  The filter answers now."""
    msg, infos = stress_dims.check_forms(oracle, acc, d, forms, 4)
    assert msg is None, (d, msg, infos)
    assert all(i["diag"]["exact_fallback_queries"] == 0 and i["diag"]["path"] == 0 for i in infos.values()), infos


# ---- through vector_scan_v1: the mirror chooses shadows and layout from dim (plugin.cpp corpus_append, view_of) -------------
def _vt(L, config):
    L.yams_plugin_shutdown()
    assert L.yams_plugin_init(config, None) == 0
    p = C.c_void_p()
    assert L.yams_plugin_get_interface(b"vector_scan_v1", 1, C.byref(p)) == 0
    return C.cast(p, C.POINTER(_lib.VectorScanV1)).contents


def _vt_search(vt, cid, q, k):
    nq, d = q.shape
    hits = C.POINTER(_lib.ScanHit)(); counts = _lib.u32p(); diag = _lib.ScanDiag()
    st = vt.search_batch_ex(None, cid, q.ctypes.data_as(_lib.f32p), nq, d, k, -1.0, 0, 0, None, C.byref(hits), C.byref(counts), C.byref(diag))
    assert st == 0, st
    cnt = [int(counts[qi]) for qi in range(nq)]
    rows = [[hits[qi * k + i].row for i in range(cnt[qi])] for qi in range(nq)]
    sims = [np.array([hits[qi * k + i].similarity for i in range(cnt[qi])], np.float32) for qi in range(nq)]
    vt.free_hits(None, hits, counts)
    return rows, sims, diag.as_dict()


@pytest.mark.parametrize("dim", [30, 100, 48, 320, 1536, 4096, 4160])
def test_vector_scan_v1_across_the_lattice(accel_lib, oracle, dim):
    """A mirror configured for the rotated layout, ragged appends, one batch of 7 and one of 140 queries: every answer is the
    oracle's; the plugin's health report counts the corpus as rotated exactly where the layout exists."""
    L = accel_lib
    vt = _vt(L, b'{"device": 0, "i8_layout": "rotated"}')
    try:
        n, k = 4200, 10
        d = dl.fixed_draw("F" if dim % 64 == 0 and dim >= 256 else "A", "default", SCAN_COSINE, dim, n=n, nq=140, k=k, seed=2000 + dim, tie=False)
        c = dl.build_case(d)
        cid = C.c_uint64()
        assert vt.corpus_create(None, dim, C.byref(cid)) == 0
        pos = 0
        for step in (1, 63, 64, 4000 - 128, 65, n):                 # ragged appends, one of them across the 4096-row mark
            step = min(step, n - pos)
            if step:
                part = np.ascontiguousarray(c.corpus[pos:pos + step])
                assert vt.corpus_append(None, cid, part.ctypes.data_as(_lib.f32p), step) == 0
                pos += step
        nn = C.c_uint64(); dd = C.c_uint32()
        assert vt.corpus_size(None, cid, C.byref(nn), C.byref(dd)) == 0 and (nn.value, dd.value) == (n, dim)
        hp = C.c_void_p()
        assert L.yams_plugin_get_health_json(C.byref(hp)) == 0
        rotated = json.loads(C.string_at(hp))["corpora_with_rotated_i8_shadow"]
        C.CDLL(None).free(hp)
        assert rotated == (1 if dl.i8_rotation_window(dim) else 0), (dim, rotated)
        many = oracle.scan_cosine_many(c.corpus, c.queries, k, -1.0)
        for nq in (7, 140):
            rows, sims, diag = _vt_search(vt, cid, np.ascontiguousarray(c.queries[:nq]), k)
            assert diag["rows_visited"] == nq * n
            for qi in range(nq):
                cnt = int(many[2][qi])
                assert rows[qi] == many[0][qi, :cnt].tolist(), (dim, nq, qi, rows[qi], many[0][qi, :cnt])
                assert np.array_equal(sims[qi].view(np.uint32), many[1][qi, :cnt].view(np.uint32)), (dim, nq, qi)
            for qi in (0, nq - 1):                                    # (the batched oracle driver against the single-query function)
                orow, osim, _, _ = oracle.scan_cosine(c.corpus, c.queries[qi], k)
                assert rows[qi] == orow.tolist() and np.array_equal(sims[qi].view(np.uint32), osim.view(np.uint32))
        assert vt.corpus_destroy(None, cid) == 0
    finally:
        L.yams_plugin_shutdown()
