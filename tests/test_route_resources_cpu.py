"""route_kernels.hip compiled for gfx950 with the product flags: every kernel keeps f32 (and f64) denormals — the kernel
descriptors' float_denorm_mode is 3, what the router's float divide of denormal norm products needs —, uses no scratch, sums
nothing with a float atomic, and the score kernels keep the waves their shared cores (row_chains.h, fp64_tile.h) are shaped for.
The float steps are there as single instructions: a rounded multiply, an add, and the scaled-divide sequence of the correctly
rounded divide; nothing is fused into an f32 fma outside that sequence's own."""
import os
import re
import shutil

import pytest

from _kernel_asm import kernel_asm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def assembly():
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.fail("hipcc is needed to compile route_kernels.hip")
    return kernel_asm("route_kernels.hip")


def test_the_seven_kernels_keep_denormals_and_use_no_scratch(assembly):
    kernels, meta, text = assembly
    assert len(kernels) == 7, sorted(kernels)      # norm, rows <1> <4> <8>, tile <vector> <scalar loads>, fold
    for name in kernels:
        desc = text.split(".amdhsa_kernel " + name)[1].split(".end_amdhsa_kernel")[0]
        assert re.findall(r"\.amdhsa_float_denorm_mode_32\s+(\d+)", desc) == ["3"], name
        assert re.findall(r"\.amdhsa_float_denorm_mode_16_64\s+(\d+)", desc) == ["3"], name
        assert re.findall(r"\.amdhsa_float_round_mode_32\s+(\d+)", desc) == ["0"], name      # round to nearest even
        assert re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", desc) == ["0"], name
        m = meta[name]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert not any("scratch_" in l for l in kernels[name]), name
        assert not any(re.search(r"atomic_(add|pk_add|fadd|max|fmax)_f(32|64)|atomic_f(add|max)", l) for l in kernels[name]), name


def test_the_score_kernels_keep_the_waves_of_their_cores(assembly):
    """512 registers per lane and SIMD, handed out in granules of 8: at most 128 leave four waves per SIMD, at most 168 three
    (tests/test_kernel_resources_cpu.py has the arithmetic).  LDS: the shared constants of row_chains.h / fp64_tile.h alone."""
    _, meta, _ = assembly
    header = open(os.path.join(ROOT, "yams_amd", "csrc", "row_chains.h")).read()
    c = {k: int(v) for k, v in re.findall(r"constexpr\s+int\s+(kRow\w+)\s*=\s*(\d+)\s*;", header)}
    for qg in (1, 4, 8):
        name = [k for k in meta if "route_score_rows_kernelILi%dEE" % qg in k]
        assert len(name) == 1, (qg, sorted(meta))
        m = meta[name[0]]
        assert m["group_segment_fixed_size"] == 4 * (c["kRowThreads"] * (c["kRowChunk"] + 1) + qg * c["kRowChunk"] + c["kRowThreads"]), (name, m)
        assert m.get("agpr_count", 0) == 0 and m["vgpr_count"] <= 128, (name, m)
    tiles = [k for k in meta if "route_score_tile_kernel" in k]
    assert len(tiles) == 2 and {("ILb1E" in k) for k in tiles} == {True, False}, tiles
    for name in tiles:
        m = meta[name]
        assert m["group_segment_fixed_size"] == 25088 and m.get("agpr_count", 0) == 0 and m["vgpr_count"] <= 168, (name, m)


def test_the_epilogue_is_the_contracts_float_steps(assembly):
    kernels, _, _ = assembly
    for name, body in kernels.items():
        if "route_score" not in name:
            continue
        assert any(re.search(r"\bv_cvt_f32_f64", l) for l in body), name                     # float(dot)
        assert any(re.search(r"\bv_div_scale_f32", l) for l in body) and any(re.search(r"\bv_div_fixup_f32", l) for l in body), name
        assert any(re.search(r"\bv_(pk_)?mul_f32", l) for l in body) and any(re.search(r"\bv_(pk_)?add_f32", l) for l in body), name
        assert any(re.search(r"\bv_fmac?_f64", l) for l in body), name                       # the chains: exact products, fma == +=
        assert not any(re.search(r"v_mfma|\bv_rcp_iflag|\bv_mac_f32|\bv_mad_f32", l) for l in body), name
