"""The dimension lattice on the CPU (tests/_dim_lattice.py, tests/stress_dims.py): the harness's dry run reaches every
counter, every localised case discriminates (the oracle alone says so), the comparison reports each mutation, and the restated
routing gives the hand-computed answer on both sides of every boundary."""
import numpy as np
import pytest

import _dim_lattice as dl
import stress_dims
from _dim_lattice import SCAN_COSINE, SCAN_L2, restated_route
from yams_amd._lib import (TIER_NONE, TIER_I8, TIER_BF16, TIER_SPLIT, TIER_F32, FLAG_FORCE_EXACT, FLAG_F32_FILTER, FLAG_SPLIT_FILTER,
                           FLAG_WIDE_TILE, FLAG_RESIDENT_QUERIES, FLAG_NO_I8_FILTER)


@pytest.fixture(scope="module")
def dry():
    seen = []
    res = stress_dims.run(dry_run=True, on_case=lambda d, msg, info: seen.append((d, msg, info)))
    return res, seen


def test_dry_run_reaches_every_counter_five_times_without_a_mismatch(dry):
    res, seen = dry
    assert "failed" not in res, res
    assert res["cases"] == stress_dims.DEFAULT_CASES == len(seen) and res["mismatches"] == 0
    short = {name: res["counters"].get(name, 0) for name in stress_dims.required_counters() if res["counters"].get(name, 0) < 5}
    assert not short, short
    # every class met every one of its dims' forms on the tier the restated route names (the tier_* counters of a dry run)
    for name in ("tier_C_f32_default", "tier_D_bf16_default", "tier_D_split_split", "tier_E_bf16_default", "tier_E_bf16_wide",
                 "tier_E_split_split", "tier_E_bf16_bare", "tier_F_i8_plain", "tier_F_i8_rotated", "tier_F_i8_resident",
                 "tier_A_none_default", "tier_B_none_default"):
        assert res["counters"].get(name, 0) >= 5, (name, res["counters"])


def test_every_localised_case_of_the_dry_run_discriminates(dry):
    """check_case returns "the case does not discriminate: ..." when discriminates() objects: no case did, and the cases held
    localised queries on every kind of group (at least three per case wherever the dim has a group)."""
    res, seen = dry
    assert all(msg is None for _, msg, _ in seen), [m for _, m, _ in seen if m]
    with_groups = [(d, info) for d, _, info in seen if d["dim"] >= 8 and d["nq"] >= 5 and info["localised"] >= 3]
    assert len(with_groups) >= 60
    assert all(d["dim"] < 8 for d, _, info in seen if info["localised"] == 0)


def test_discriminates_reports_a_case_whose_group_does_not_matter(oracle):
    """The check itself bites: a localised case whose planted rows are replaced by random ones is reported."""
    d = dl.fixed_draw("E", "default", SCAN_COSINE, 256, n=4096, nq=4, k=10)
    c = dl.build_case(d)
    assert dl.discriminates(oracle, c) is None
    rng = np.random.default_rng(1)
    for rows in c.planted.values():
        c.corpus[rows] = rng.standard_normal((len(rows), 256)).astype(np.float32)
    assert dl.discriminates(oracle, c) is not None


@pytest.mark.parametrize("cls", list(dl.CLASSES))
def test_scripted_device_cases_discriminate(oracle, cls):
    """The scripted cells of tests/test_dim_lattice_gpu.py, rehearsed: every one of their localised queries discriminates."""
    for dim in dl.CLASSES[cls]:
        for metric, forms, l2_acc, limit, d in stress_dims.scripted_draws(cls, dim):
            c = dl.build_case(d)
            assert dl.discriminates(oracle, c) is None, (cls, dim, metric)
            assert forms and (dim < 8 or len(c.localised) >= min(3, (d["nq"] + 1) // 2, max(1, dl.group(dim, "first")[1])))


def test_scripted_masked_planner_and_filter_pass_cases_discriminate(oracle):
    for d, forms in stress_dims.masked_draws() + stress_dims.planner_draws() + stress_dims.filter_pass_draws():
        c = dl.build_case(d)
        assert dl.discriminates(oracle, c) is None, d
        n_allowed = None if c.allowed is None else len(c.allowed)
        assert (n_allowed is None or n_allowed >= 16384) and dl.route(d, n_allowed) == (0, TIER_I8 if d["cls"] == "F" else TIER_BF16), (d, n_allowed)


def test_self_test_reports_every_mutation(oracle):
    assert stress_dims.self_test(oracle) == []


def test_groups_lie_where_the_design_says():
    assert dl.group(8176, "tail") == (8160, 16) and dl.group(8192, "tail") == (8176, 16) and dl.group(100, "tail") == (96, 4)
    assert dl.group(37, "tail") == (32, 5) and dl.group(4032, "straddle_P") == (2040, 16) and dl.group(4096, "straddle_P") is None
    assert dl.group(8176, "last32") == (8128, 16) and dl.group(8176, "last64") == (8088, 16) and dl.group(5, "first") is None
    for cls, dims in dl.CLASSES.items():
        for dim in dims:
            for kind in dl.G_KINDS:
                g = dl.group(dim, kind)
                assert g is None or (0 <= g[0] and g[0] + g[1] <= dim and 1 <= g[1] <= 16 and dim - g[1] >= 3), (dim, kind, g)
    assert dl.walk(768, True) == "staged" and dl.walk(100, True) == "vec4_tail" and dl.walk(100, False) == "scalar" and dl.walk(37, True) == "scalar"
    assert [dl.i8_rotation_window(x) for x in (192, 256, 320, 4032, 4096, 4160)] == [0, 256, 256, 2048, 4096, 0]


BF, I8, BOTH = {"bf16"}, {"i8"}, {"bf16", "i8"}


@pytest.mark.parametrize("args,want", [
    # (dim, aligned, shadows, nq, k, metric, flags, n, n_allowed) -> (path, filter_tier), computed by hand from scan_api.cpp
    ((3, True, set(), 17, 10, SCAN_COSINE, 0, 4096, None), (1, TIER_NONE)),        # dim % 4 != 0: exhaustive
    ((4, True, BF, 17, 10, SCAN_COSINE, 0, 4096, None), (0, TIER_F32)),             # dim % 4 == 0, % 16 != 0: the f32 tier
    ((12, True, BF, 17, 10, SCAN_COSINE, 0, 4096, None), (0, TIER_F32)),
    ((16, True, BF, 17, 10, SCAN_COSINE, 0, 4096, None), (0, TIER_BF16)),           # dim % 16 == 0: bf16
    ((48, True, BF, 1, 10, SCAN_COSINE, 0, 4096, None), (0, TIER_BF16)),            # one query, but dim % 32 != 0: not fused
    ((64, True, BF, 1, 10, SCAN_COSINE, 0, 4096, None), (1, TIER_NONE)),            # ... dim % 32 == 0: the fused small scan
    ((64, True, BF, 17, 10, SCAN_COSINE, 0, 4096, None), (0, TIER_BF16)),
    ((240, True, I8, 17, 10, SCAN_COSINE, 0, 4096, None), (0, TIER_BF16)),          # the int8 tier needs dim % 64 == 0, dim >= 256
    ((256, True, I8, 17, 10, SCAN_COSINE, 0, 4096, None), (0, TIER_I8)),
    ((192, True, I8, 17, 10, SCAN_COSINE, 0, 4096, None), (0, TIER_BF16)),
    ((512, True, I8, 200, 10, SCAN_COSINE, FLAG_RESIDENT_QUERIES, 5001, None), (0, TIER_I8)),
    ((544, True, I8, 200, 10, SCAN_COSINE, FLAG_RESIDENT_QUERIES, 5001, None), (0, TIER_BF16)),
    ((768, True, I8, 1, 10, SCAN_COSINE, 0, 4096, None), (1, TIER_NONE)),           # fused: dim <= 1024, one query
    ((768, True, I8, 1, 100, SCAN_COSINE, 0, 4096, None), (0, TIER_I8)),            # 16 workgroups x 100 survivors > 1024
    ((832, True, I8, 17, 10, SCAN_COSINE, 0, 4096, None), (0, TIER_I8)),
    ((768, True, BOTH, 128, 10, SCAN_COSINE, 0, 4096, None), (0, None)),            # both shadows, <= 128 queries, the resident form's last dim: the CU count decides
    ((832, True, BOTH, 128, 10, SCAN_COSINE, 0, 4096, None), (0, TIER_BF16)),       # ... above R_MAX_SLABS slabs no resident form: the narrow bf16 form keeps the batch
    ((896, True, BOTH, 128, 10, SCAN_COSINE, 0, 4096, None), (0, TIER_BF16)),       # (% 128 == 0, but above 768)
    ((512, True, BOTH, 64, 10, SCAN_COSINE, 0, 4096, None), (0, None)),             # 512: the persistent bf16 form's last dim and a resident dim
    ((544, True, BOTH, 64, 10, SCAN_COSINE, 0, 4096, None), (0, TIER_BF16)),        # 544: neither (no int8 shadow can exist: % 64 != 0)
    ((448, True, BOTH, 64, 10, SCAN_COSINE, 0, 4096, None), (0, TIER_BF16)),        # % 64 == 0 but % 128 != 0: no resident form
    ((448, True, BOTH, 129, 10, SCAN_COSINE, 0, 4096, None), (0, TIER_I8)),
    ((1536, True, BOTH, 64, 10, SCAN_L2, 0, 4096, None), (0, TIER_BF16)),
    ((832, True, BOTH, 129, 10, SCAN_COSINE, 0, 4096, None), (0, TIER_I8)),
    ((1024, True, BF, 16, 10, SCAN_COSINE, 0, 4096, None), (1, TIER_NONE)),         # the fused scan's last dim
    ((1056, True, BF, 16, 10, SCAN_COSINE, 0, 4096, None), (0, TIER_BF16)),         # ... and the first it refuses
    ((1024, True, BF, 17, 10, SCAN_COSINE, 0, 4096, None), (0, TIER_BF16)),
    ((4096, True, I8, 17, 10, SCAN_COSINE, 0, 4096, None), (0, TIER_I8)),
    ((4160, True, I8, 17, 10, SCAN_COSINE, 0, 4096, None), (0, TIER_I8)),           # (no rotated layout there; the plain one scans)
    ((64, False, set(), 17, 10, SCAN_COSINE, 0, 5001, None), (1, TIER_NONE)),       # a misaligned base: exhaustive although n >= 4096
    ((64, True, set(), 17, 10, SCAN_COSINE, 0, 5001, None), (0, TIER_BF16)),        # (a bare view: the k32 kernel, the same tier)
    ((64, True, BF, 17, 10, SCAN_COSINE, 0, 4095, None), (1, TIER_NONE)),           # below kMfmaMinRows
    ((64, True, BF, 17, 10, SCAN_COSINE, 0, 5001, 4000), (1, TIER_NONE)),           # an allow-mask below 16384 rows is gathered
    ((64, True, BF, 17, 10, SCAN_COSINE, 0, 20000, 16384), (0, TIER_BF16)),
    ((64, True, BF, 17, 10, SCAN_COSINE, FLAG_FORCE_EXACT, 5001, None), (1, TIER_NONE)),
    ((64, True, BF, 17, 10, SCAN_COSINE, FLAG_F32_FILTER, 5001, None), (0, TIER_F32)),
    ((64, True, BF, 17, 10, SCAN_COSINE, FLAG_SPLIT_FILTER, 5001, None), (0, TIER_SPLIT)),
    ((64, True, BF, 1, 10, SCAN_COSINE, FLAG_WIDE_TILE, 5001, None), (0, TIER_BF16)),   # a named form keeps off the fused scan
    ((256, True, I8, 17, 10, SCAN_COSINE, FLAG_NO_I8_FILTER, 4096, None), (0, TIER_BF16)),
    ((256, True, I8, 17, 10, SCAN_COSINE, FLAG_SPLIT_FILTER, 4096, None), (0, TIER_SPLIT)),
    ((64, True, BF, 17, 661, SCAN_COSINE, 0, 5001, None), (0, TIER_BF16)),          # 3 k + 64 = 2047 <= 2048
    ((64, True, BF, 17, 662, SCAN_COSINE, 0, 5001, None), (0, TIER_SPLIT)),
    ((64, True, BF, 17, 320, SCAN_L2, 0, 5001, None), (0, TIER_BF16)),              # 6 k + 128 = 2048
    ((64, True, BF, 17, 321, SCAN_L2, 0, 5001, None), (0, TIER_SPLIT)),
    ((64, True, BF, 1, 10, SCAN_L2, 256, 4096, None), (0, TIER_BF16)),              # fp32 accumulation keeps L2 off the fused scan
    ((64, True, BF, 1, 10, SCAN_L2, 0, 4096, None), (1, TIER_NONE)),
    ((768, True, BOTH, 129, 10, SCAN_L2, 0, 4096, None), (0, TIER_I8)),             # L2 on the int8 tier needs the norms of the bf16 shadow
    ((768, True, BOTH, 128, 10, SCAN_L2, 0, 4096, None), (0, None)),
    ((768, True, I8, 129, 10, SCAN_L2, 0, 4096, None), (0, TIER_BF16)),
])
def test_restated_route_on_both_sides_of_every_boundary(args, want):
    assert restated_route(*args) == want
